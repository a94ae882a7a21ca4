"""Phase-field fracture of a notched plate under load stepping with the latent variable proximal point method on the HIP
backend.  Counterpart of the reference's examples/03_fracture/fracture_dolfinx.py, with its command line.  One difference: the
reference parses --res and then meshes with max_res=0.0125 regardless (:78); here --res is honoured.  Output: u, c, psi
(solution_*.vtu) and ConformingDamage (damage_*.vtu) every --write-frequency load steps, and attempts.npz with the log of all
attempts and the per-step Newton and LVPP counts."""
import sys
import time
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from proximalgalerkin_amd.fracture import solve_problem  # noqa: E402


def main(argv=None):
    parser = ArgumentParser(description="Phase-field fracture of a notched plate, proximal Galerkin, on the GPU.",
                            formatter_class=ArgumentDefaultsHelpFormatter)
    parser.add_argument("--res", "-r", dest="res", type=float, default=0.0125, help="Resolution of the mesh")
    parser.add_argument("--max-fail-iter", type=int, default=50, dest="NFAIL_MAX",
                        help="Maximum number of iterations of the LVPP that can fail before termination")
    parser.add_argument("--write-frequency", type=int, default=25, dest="write_frequency", help="Frequency of writing output")
    parser.add_argument("--num-load-steps", type=int, default=1001, dest="num_load_steps", help="Number of load steps")
    parser.add_argument("--verbose", "-v", action="store_true", help="Verbose output from the Newton solver")
    parser.add_argument("--Tmin", type=float, default=0.0, help="Minimum load")
    parser.add_argument("--Tmax", type=float, default=5.0, help="Maximum load")
    parser.add_argument("--result_dir", type=Path, default=Path("output"), help="Directory to store results")
    a = parser.parse_args(argv)
    from proximalgalerkin_amd.fracture import SP

    sp = dict(SP)
    if a.verbose:
        sp.update({"snes_monitor": None, "snes_linesearch_monitor": None})
    t0 = time.perf_counter()
    log, newton_its, lvpp_its = solve_problem(res=a.res, num_load_steps=a.num_load_steps, Tmin=a.Tmin, Tmax=a.Tmax,
                                              nfail_max=a.NFAIL_MAX, write_frequency=a.write_frequency, result_dir=a.result_dir,
                                              verbose=True, petsc_options=sp)
    print(f"wall time {time.perf_counter() - t0:.2f} s, load steps {len(newton_its)}, attempts {len(log)}, "
          f"Newton iterations {int(newton_its.sum())}, LVPP iterations {int(lvpp_its.sum())}", flush=True)
    a.result_dir.mkdir(parents=True, exist_ok=True)
    np.savez(a.result_dir / "attempts.npz", log=log, newton_its=newton_its, lvpp_its=lvpp_its, res=a.res,
             num_load_steps=a.num_load_steps, Tmin=a.Tmin, Tmax=a.Tmax)


if __name__ == "__main__":
    main()
