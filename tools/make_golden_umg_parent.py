#!/usr/bin/env python3
"""Records tests/golden/umg_d34_parent.npz: the finest mesh of D34 (tests/umg_reference.py) solved by the PARENT commit, which has no
hierarchies - what a handle without one must still do, bit for bit (tests/test_gpu_umg.py).

    python3 tools/make_golden_umg_parent.py <checkout of the parent commit, built> <parent commit id> [outdir]

The mesh comes from this tree (the parent has no fem.refine) and is stored in the file; the solves - settings B under "pgx_lu" and under
"pgx_mg", each twice, which must agree bitwise - run in a child process that imports the parent's package.  Needs an MI355X."""
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
BASE = {"ksp_type": "preonly", "ksp_error_if_not_converged": True, "snes_error_if_not_converged": True, "snes_linesearch_type": "none",
        "snes_rtol": 1e-6, "snes_max_it": 100}


def solve_with(parent_dir, mesh_file, out_file):
    sys.path.insert(0, parent_dir)
    from proximalgalerkin_amd import fem
    from proximalgalerkin_amd.obstacle import run_outer_loop, setup_problem

    assert pathlib.Path(fem.__file__).resolve().is_relative_to(pathlib.Path(parent_dir).resolve()), fem.__file__
    m = np.load(mesh_file)
    rec = dict(coords=m["coords"], cells=m["cells"])
    for tag, pc in (("lu", "pgx_lu"), ("mg", "pgx_mg")):
        runs = []
        for _ in range(2):
            problem, sol, sol_k, alpha = setup_problem(fem.Mesh(m["coords"], m["cells"]), 1, petsc_options=dict(BASE, pc_type=pc))
            lin, solve = [], problem.solve

            def counted():
                r = solve()
                lin.append(problem.solver.getLinearSolveIterations())
                return r

            problem.solve = counted
            hist = run_outer_loop(problem, sol, sol_k, alpha, 500, "double_exponential", 1e2, 1e-4)
            runs.append((sol.x.array[: len(m["coords"])].copy(), [int(v) for v in hist["Newton steps"]], list(lin)))
            problem.close()
        (u, newton, lin), (u2, newton2, lin2) = runs
        assert newton == newton2 and lin == lin2 and u.tobytes() == u2.tobytes(), (tag, newton, newton2, lin, lin2)
        print(f"{tag}: Newton {newton}, Krylov {lin}", flush=True)
        rec.update({f"u_{tag}": u, f"newton_{tag}": np.array(newton, dtype=np.int32), f"linear_{tag}": np.array(lin, dtype=np.int32)})
    np.savez_compressed(out_file, **rec)


def main():
    if sys.argv[1] == "--solve":
        return solve_with(*sys.argv[2:5])
    parent_dir, commit = str(pathlib.Path(sys.argv[1]).resolve()), sys.argv[2]
    assert len(commit) == 40, "the full id of the commit the parent checkout was built from"
    out = pathlib.Path(sys.argv[3]) if len(sys.argv) > 3 else ROOT / "tests" / "golden"
    out.mkdir(parents=True, exist_ok=True)
    sys.path.insert(0, str(ROOT))
    from tests import umg_reference as UR

    msh = UR.build_mesh("D34")
    with tempfile.TemporaryDirectory() as tmp:
        mesh_file = str(pathlib.Path(tmp) / "mesh.npz")
        np.savez(mesh_file, coords=msh.geometry, cells=msh.cells)
        tmp_out = str(pathlib.Path(tmp) / "out.npz")
        subprocess.run([sys.executable, __file__, "--solve", parent_dir, mesh_file, tmp_out], check=True, cwd=parent_dir)
        rec = dict(np.load(tmp_out))
    rec["parent_commit"] = np.array(commit)
    np.savez_compressed(out / "umg_d34_parent.npz", **rec)
    print(f"wrote {out / 'umg_d34_parent.npz'}")


if __name__ == "__main__":
    main()
