"""The eikonal equation on a Moebius strip, latent variable proximal point method on the HIP backend.  Counterpart of the reference's
examples/09_eikonal/eikonal_dolfinx.py.  The strip is meshed natively from its parametrisation (nu x nv curved quadrilaterals of
geometry order `--order`); reading the ParaView VTU that MFEM writes (the script's --mesh-dir) is NOT supported, and the facet-normal
point cloud of the script is left out.  Output: the prints of the script, eikonal.vtu with the DG fields u, grad(u) and psi (in place of
u.bp and psi.bp) and steps.npz with the log of the LVPP steps."""
import sys
import time
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from proximalgalerkin_amd.eikonal import TOL, solve_problem, solver_parameters  # noqa: E402


def main(argv=None):
    parser = ArgumentParser(description="Eikonal equation on a Moebius strip, proximal Galerkin, on the GPU.  The mesh is generated "
                            "from the strip's parametrisation; the reference's --mesh-dir (an MFEM ParaView VTU) is not read.",
                            formatter_class=ArgumentDefaultsHelpFormatter)
    parser.add_argument("--nu", type=int, default=64, help="Cells around the strip (>= 3)")
    parser.add_argument("--nv", type=int, default=8, help="Cells across the strip")
    parser.add_argument("--order", type=int, default=3, help="Geometry order of the cells (1, 2 or 3)")
    parser.add_argument("--nq1", type=int, default=6, help="Gauss points per direction (1..11)")
    parser.add_argument("--scale", type=float, default=1.0, help="Radius of the centre circle; the strip's half-width is scale / 4")
    parser.add_argument("--tol", type=float, default=TOL, help="The script's tol: SNES tolerances, and 5 tol stops the loop")
    parser.add_argument("--verbose", "-v", action="store_true", help="Verbose output from the Newton solver")
    parser.add_argument("--result_dir", type=Path, default=Path("output"), help="Directory to store results")
    parser.add_argument("--linear-solver", choices=("dense", "banded"), default="dense",
                        help="LU with partial pivoting of the Newton matrix: dense (at most 32768 unknowns) or banded in the folded order")
    parser.add_argument("--profile", type=Path, default=None, nargs="?", const=Path("auto"),
                        help="Write the timing split of the run to this JSON file (no value: profiles/ex09_nu<nu>_nv<nv>[_banded].json)")
    a = parser.parse_args(argv)
    sp = solver_parameters(a.tol)
    if a.verbose:
        sp.update({"snes_monitor": None, "snes_linesearch_monitor": None})
    prof = {} if a.profile is not None else None
    t0 = time.perf_counter()
    fields, log = solve_problem(nu=a.nu, nv=a.nv, order=a.order, nq1=a.nq1, scale=a.scale, tol=a.tol, snes_opts=sp, profile=prof,
                                result_dir=a.result_dir, verbose=True, linear_solver=a.linear_solver)
    wall = time.perf_counter() - t0
    unknowns = len(fields["u"]) + fields["psi"].size
    print(f"wall time {wall:.2f} s, {unknowns} unknowns, max u {fields['u'].max():.6f}, max |psi| {np.abs(fields['psi']).max():.4f}", flush=True)
    a.result_dir.mkdir(parents=True, exist_ok=True)
    np.savez(a.result_dir / "steps.npz", log=log, nu=a.nu, nv=a.nv, order=a.order, nq1=a.nq1, scale=a.scale, tol=a.tol)
    if a.profile is not None:
        import json

        path = a.profile
        if str(path) == "auto":
            path = Path(__file__).resolve().parents[2] / "profiles" / f"ex09_nu{a.nu}_nv{a.nv}{'_banded' if a.linear_solver == 'banded' else ''}.json"
        ms = {k: v for k, v in prof.items() if k not in ("lu", "band")}
        steps = int(log[:, 2].sum())
        out = dict(nu=a.nu, nv=a.nv, order=a.order, nq1=a.nq1, scale=a.scale, unknowns=unknowns, lvpp_iterations=len(log),
                   newton_iterations=steps, wall_s=wall, ms=ms,
                   lu_factor_share_of_newton=ms["lu_factor"] / ms["newton_total"] if ms["newton_total"] > 0 else None, lu=prof["lu"],
                   linear_solver=a.linear_solver)
        if "band" in prof:  # flops of a band factorisation counted as 2 n kl (kl + ku)
            b = prof["band"]
            out["band"] = b
            out["lu_factor_flops_each"] = 2.0 * b["n"] * b["kl"] * (b["kl"] + b["ku"])
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
