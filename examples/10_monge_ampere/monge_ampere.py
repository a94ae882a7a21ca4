"""The Monge-Ampere equation through a three-field mixed discretisation with the matrix logarithm of the Hessian as latent variable, on
the HIP backend.  Counterpart of the reference's examples/10_monge_ampere/monge_ampere_dolfinx.py, which takes no arguments: the default
is its p-refinement study (k = 3 ... 14 on the 2 x 2 mesh of [-1, 1]^2, each degree warm-started from the one before); `--study h`
runs the script with its commented-out `refine` line enabled (one degree, n doubling).  Output: the errors the script prints, and
solution.vtu with the last u on the dof lattice (in place of the script's solution_{j}.bp)."""
import sys
import time
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from proximalgalerkin_amd import io, lagrange  # noqa: E402
from proximalgalerkin_amd.monge_ampere import SP, h_refinement, p_refinement, write_profile  # noqa: E402


def write_u(path: Path, problem, z):
    """u at the P_k nodes, every cell split into the k^2 triangles of its node lattice"""
    k = problem.k
    ref = np.rint(lagrange.lattice(k) * k).astype(int)
    loc = {(i, j): a for a, (i, j) in enumerate(map(tuple, ref))}
    sub = [(loc[i, j], loc[i + 1, j], loc[i, j + 1]) for j in range(k) for i in range(k - j)]
    sub += [(loc[i + 1, j], loc[i + 1, j + 1], loc[i, j + 1]) for j in range(k - 1) for i in range(k - 1 - j)]
    tri = problem.cell_dofs_u[:, np.array(sub)].reshape(-1, 3).astype(np.int32)
    path.parent.mkdir(parents=True, exist_ok=True)
    io.write_vtu(path, problem.Xu, tri, point_data={"u": z[:problem.nu]})


def main(argv=None):
    parser = ArgumentParser(description="Monge-Ampere, three-field mixed method with a log-Hessian latent variable, on the GPU.",
                            formatter_class=ArgumentDefaultsHelpFormatter)
    parser.add_argument("--study", choices=("p", "h"), default="p", help="p: degrees k-min .. k-max on one mesh; h: one degree, n doubling")
    parser.add_argument("--k-min", type=int, default=3, dest="k_min")
    parser.add_argument("--k-max", type=int, default=14, dest="k_max")
    parser.add_argument("-n", type=int, default=2, help="Cells per direction (p-study)")
    parser.add_argument("-k", type=int, default=4, help="Degree (h-study)")
    parser.add_argument("--levels", type=int, nargs="+", default=[2, 4, 8], help="Cells per direction of the h-study")
    parser.add_argument("--nonsmooth", action="store_true", help="The script's nonsmooth data")
    parser.add_argument("--verbose", "-v", action="store_true", help="Verbose output from the Newton solver")
    parser.add_argument("--result_dir", type=Path, default=Path("output"), help="Directory to store results")
    parser.add_argument("--profile", type=Path, default=None, help="Write the timing split of the run to this JSON file")
    a = parser.parse_args(argv)
    sp = dict(SP)
    if a.verbose:
        sp.update({"snes_monitor": None, "snes_linesearch_monitor": None})
    prof = {} if a.profile is not None else None
    t0 = time.perf_counter()
    kw = dict(nonsmooth=a.nonsmooth, snes_opts=sp, profile=prof, verbose=True, return_last=True)
    out = p_refinement(a.k_min, a.k_max, a.n, **kw) if a.study == "p" else h_refinement(a.k, tuple(a.levels), **kw)
    wall = time.perf_counter() - t0
    print("Errors", out["errors"], flush=True)
    print(f"wall time {wall:.2f} s, unknowns per level {out['ndofs']}, Newton steps {out['newton_its']}", flush=True)
    write_u(a.result_dir / "solution.vtu", out["problem"], out["states"][-1])
    out["problem"].close()
    if a.profile is not None:
        prof.update(study=a.study, nonsmooth=a.nonsmooth, wall_s=wall, errors=out["errors"], newton_its=out["newton_its"],
                    reasons=out["reasons"])
        write_profile(a.profile, prof)


if __name__ == "__main__":
    main()
