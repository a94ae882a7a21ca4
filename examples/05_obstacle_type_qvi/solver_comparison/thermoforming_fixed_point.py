"""Thermoforming quasi-variational inequality by a fixed point in the mould temperature, with a Moreau-Yosida path for the
membrane, on the HIP backend.  Counterpart of the reference's
examples/05_obstacle_type_qvi/solver_comparison/thermoforming_fixed_point.jl (a script without flags; -M sets the mesh size
the reference hard-codes as 150, --max-newton NLsolve's iteration cap, --max-outer the length of its outer loop).  The last
line printed is the reference's: run time, fixed point iterations, linear system solves."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))
from proximalgalerkin_amd.thermoforming_comparison import solve_fixed_point  # noqa: E402

if __name__ == "__main__":
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("-M", type=int, default=150, help="cells per side of the unit square")
    parser.add_argument("--max-newton", type=int, default=1000, help="Newton iterations per solve (NLsolve's default)")
    parser.add_argument("--max-outer", type=int, default=10_000, help="fixed point iterations")
    a = parser.parse_args()
    solve_fixed_point(a.M, max_newton=a.max_newton, max_outer=a.max_outer)
